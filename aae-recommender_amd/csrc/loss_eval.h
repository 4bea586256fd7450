// The loss of a model on rows it was not trained on (reference vae.py:243-264: loss_function on every test batch; aae.py:176-177,
// 693-695: F.binary_cross_entropy(x_hat + TINY, target + TINY)): per row the SUM over the N items of the cell loss, and for
// the VAE the row's KL term - without the [rows, n_items] matrix wherever the fused rank kernels apply.
//
//   fused form (handles with rank_ok / vae_rank_ok), behind the gather, the chain program and known_mask_kernel of a fused
//   ranking call (abi_rank.h) - the mask here is the bitmap of the rows' TARGET entries:
//     1. rank_x3_kernel<.., kRankLoss>   every cell whose bit is clear adds loss_cell_t0(logit) (rank_x3.h): four cells of a
//                                        tile in fp32, onto the thread's fp64 sum; per (row, workgroup) one store into lpart.
//                                        A target cell adds NOTHING.
//     2. loss_targets_kernel             one wave per target entry recomputes that logit as the (h + 1)-long dot product of the
//                                        row's dh2 with the item's row of dec.lin3 (bf16 handles: both operands rounded to
//                                        bf16 first, the products in fp32 - what that handle's matrix cores multiply) and
//                                        adds loss_cell_target(logit, value); per (row, chunk of entries) one fp64 sum.
//     3. loss_finish_kernel              row_bce[row] = sum_w lpart[row][w] in workgroup order + the chunk sums in order.
//   Why target cells are skipped and not corrected: summing every cell as zero-target and letting the fix-up subtract the
//   zero-target loss of ITS logit puts two slightly different logits of the same cell (matrix-core tile sum / wave dot
//   product) on either side of the 24 ln 2 cut-off, where the zero-target loss jumps from 16.6 to 100: such a cell would be
//   wrong by ~83.  Skipped, every cell is charged exactly once, from one logit.
//
//   dense form (every other handle; rows beyond the fused call's limit): the LOGITS of the rows (linear_fwd with EpiStore)
//   in the [max_batch][n_items] scratch, then
//     loss_rows_dense_kernel             one workgroup per row: the row's target entries first - loss_cell_target of the stored
//                                        logit, and the cell is overwritten with a marker -, then loss_cell_t0 of every
//                                        cell that carries no marker.  The same two cell functions; nothing is recovered
//                                        from a sigmoid.
//   vae_kl_rows_kernel                   row_kl[row] = -0.5 sum_c (1 + logvar - mu^2 - exp(logvar)) from the [mu | logvar]
//                                        block of the hidden half: cell terms in fp32, the row's sum in fp64, column order.
// Every sum has a fixed order for a given call shape: no float atomics, the results do not vary from run to run.
#pragma once
#include "rank_x3.h"

namespace aae {

constexpr int kLossChunk = 64;          // target entries of a row per chunk of loss_targets_kernel ...
constexpr int kLossChunksMax = 16;      // ... and the most chunks a row is cut into (longer rows: every chunk takes more)

__device__ __forceinline__ float loss_bf16_rne(float x) {      // round-to-nearest-even to bf16, as x3_split_pair's first term
    unsigned u = __float_as_uint(x);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return __uint_as_float(u & 0xFFFF0000u);
}

// the fixed-order sum of a 256-thread workgroup's fp64 values: lanes of a wave by xor shuffles, then the four waves in order
__device__ __forceinline__ double loss_block_sum(double v, double* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// grid (rows, chunks): chunk y takes entries [lo + y * per, lo + (y + 1) * per) of the row, per = ceil(entries / chunks)
// rounded up to a whole number of kLossChunk; its four waves take them round robin, each wave adds its entries in order
__global__ __launch_bounds__(256) void loss_targets_kernel(BatchView tv, const float* __restrict__ dh2, int ldh,
                                                           const float* __restrict__ V3a, int ldv, int kdim, int n_items,
                                                           int one_term, double* __restrict__ csum) {
    __shared__ double red[4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int dc = tv.doc(row);
    const int64_t lo = tv.indptr[dc], hi = tv.indptr[dc + 1];
    const int64_t per = ((hi - lo + (int64_t)gridDim.y * kLossChunk - 1) / ((int64_t)gridDim.y * kLossChunk)) * kLossChunk;
    const int64_t c_lo = lo + per * blockIdx.y, c_hi = c_lo + per < hi ? c_lo + per : hi;
    const float* x = dh2 + (size_t)row * ldh;
    double sum = 0.0;
    for (int64_t e = c_lo + wave; e < c_hi; e += 4) {
        const int n = tv.indices[e];
        if (n < 0 || n >= n_items) continue;            // (wave-uniform)
        const float* w = V3a + (size_t)n * ldv;
        float acc = 0.f;
        for (int k = lane; k < kdim; k += 64) {
            float xa = x[k], wa = w[k];
            if (one_term) { xa = loss_bf16_rne(xa); wa = loss_bf16_rne(wa); }
            acc += xa * wa;
        }
        acc = wave_sum(acc);
        sum += (double)loss_cell_target(acc, tv.values[e]);
    }
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    if (tid == 0) csum[(size_t)row * gridDim.y + blockIdx.y] = (red[0] + red[1]) + (red[2] + red[3]);
}

// one thread per row
__global__ __launch_bounds__(256) void loss_finish_kernel(const double* __restrict__ lpart, int wgs, const double* __restrict__ csum,
                                                          int chunks, int rows, double* __restrict__ row_bce) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    double s = 0.0;
    for (int w = 0; w < wgs; ++w) s += lpart[(size_t)row * wgs + w];
    for (int c = 0; c < chunks; ++c) s += csum[(size_t)row * chunks + c];
    row_bce[row] = s;
}

// one wave per row (4 rows per workgroup): mulv [rows][ld] = [mu | logvar], nc columns each
__global__ __launch_bounds__(256) void vae_kl_rows_kernel(const float* __restrict__ mulv, int ld, int nc, int rows,
                                                          double* __restrict__ row_kl) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* r = mulv + (size_t)row * ld;
    double s = 0.0;
    for (int c0 = 0; c0 < nc; c0 += 64) {               // 64 columns at a time: lane sums in a fixed tree, the groups in order
        const int c = c0 + lane;
        float t = 0.f;
        if (c < nc) { const float mu = r[c], lv = r[nc + c]; t = -0.5f * (1.f + lv - mu * mu - expf(lv)); }
        double d = (double)t;
        for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
        s += d;
    }
    if (lane == 0) row_kl[row] = s;
}

// the marker of a cell that a target entry has charged: a NaN no product yields (its payload)
constexpr unsigned kLossMarked = 0x7FC0A55Au;

// One workgroup per row of the logit matrix: row `blockIdx.x` of it is row `blockIdx.x` of the call (`tv`: its target rows).
// The target cells are overwritten with the marker.
__global__ __launch_bounds__(256) void loss_rows_dense_kernel(float* __restrict__ logits, int ld, int n_items, BatchView tv,
                                                              double* __restrict__ row_bce) {
    __shared__ double red[4];
    const int row = blockIdx.x, tid = threadIdx.x;
    float* lg = logits + (size_t)row * ld;
    const int dc = tv.doc(row);
    const int64_t lo = tv.indptr[dc], hi = tv.indptr[dc + 1];
    double sum = 0.0;
    for (int64_t e = lo + tid; e < hi; e += 256) {
        const int n = tv.indices[e];
        if (n < 0 || n >= n_items) continue;
        const float l = lg[n];
        if (__float_as_uint(l) == kLossMarked) continue;        // (an item stored twice: charged once)
        sum += (double)loss_cell_target(l, tv.values[e]);
        lg[n] = __uint_as_float(kLossMarked);
    }
    __syncthreads();
    for (int i = tid; i < n_items; i += 256) {
        const float l = lg[i];
        if (__float_as_uint(l) != kLossMarked) sum += (double)loss_cell_t0(l);
    }
    const double total = loss_block_sum(sum, red);
    if (tid == 0) row_bce[row] = total;
}

}  // namespace aae
