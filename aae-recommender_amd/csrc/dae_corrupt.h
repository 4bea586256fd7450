// DenoisingAutoEncoder's corruption drawn from the device generator (device_common.h): two streams of the one
// counter generator, so that `seed` determines a DAE run as it determines every other model's.
//   stream 13  zero corruption (reference dae.py:48-52): entry (r, j) of a CSR matrix is kept iff word(seed, step, 13, r, j) >=
//              keep_threshold(p) - the dropout rule, p the DROP probability; r = the row's index in the matrix handed over, j the item
//              id, step = *step_ctr + 1: the first training step that will read the thinned matrix (dae_thin_kernel);
//   stream 14  Gauss corruption (dae.py:40-45): cell (r, j) of the step's batch is scale * draw_gauss(key of stream 14, r, j), the
//              product in fp32; r = the row of the GLOBAL batch as dropout places it (aae_set_rng_rows), step = the opened step's value
//              (dense_noise_gen_kernel / dense_noise_finish_kernel: the noisy dense encoder input without a noise matrix in memory).
#pragma once
#include "kernels.h"

namespace aae {

constexpr uint32_t kDaeZeroStream = 13, kDaeGaussStream = 14;
constexpr int kDaeChunksMax = 64;       // column chunks (workgroups) a row of the dense input is spread over, at most

__device__ __forceinline__ uint64_t dae_stream_key(uint64_t seed, uint64_t step, uint32_t sid) {
    return rng_key(seed, step, 0) ^ ((uint64_t)sid * 0xA0761D6478BD642Full);
}

// out[e] = keep(e) ? values[e] : 0 over the entries of rows [0, n_rows).  Groups of L lanes walk the rows (L = 4 .. 64, the power of
// two at or above the matrix's mean row length, read from indptr on the device: the same for every thread), a group's lanes stride
// over its row's entries - a fixed grid whatever n_rows is, a million short rows keep 16 rows in a wave, a row longer than any
// stride is a longer loop.  Every entry is read and written by one thread: out == values is allowed.
__global__ __launch_bounds__(256) void dae_thin_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                       const float* values, int64_t n_rows, uint32_t keep_threshold, int enabled,
                                                       uint64_t seed, const long long* __restrict__ step_ctr, float* out) {
    const uint64_t key = dae_stream_key(seed, (uint64_t)(*step_ctr + 1), kDaeZeroStream);
    const int64_t nnz = indptr[n_rows] - indptr[0];
    const int64_t mean = (nnz + n_rows - 1) / n_rows;
    int shift = 2;
    while (shift < 6 && (1 << shift) < mean) ++shift;
    const int L = 1 << shift;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (int64_t)gridDim.x * blockDim.x;
    const int sub = (int)(tid & (L - 1));
    for (int64_t r = tid >> shift; r < n_rows; r += nthreads >> shift) {
        const int64_t lo = indptr[r], hi = indptr[r + 1];
        for (int64_t e = lo + sub; e < hi; e += L) {
            const float v = values[e];
            const bool keep = !enabled || hash_cell(key, (uint32_t)r, (uint32_t)indices[e]) >= keep_threshold;
            out[e] = keep ? v : 0.f;
        }
    }
}

// cell (grow, col) of the step's noise.  2 col + 1 < 2^32 for every supported n_items (n_items is an int32: 2 col + 1 <= 2^32 - 3),
// so draw_gauss's column words 2 col and 2 col + 1 never wrap.  The product is a rounded fp32 product wherever it is inlined.
__device__ __forceinline__ float dae_noise_cell(uint64_t k, uint32_t grow, int col, float scale) {
    return __fmul_rn(scale, draw_gauss(k, grow, col));
}

// The dense noisy encoder input X [rows][ldx] of a step, drawn instead of read (the sibling of dense_input_kernel):
//   X[b][n] = scale * gauss(b, n) + the batch's row b, L1-normalised over all N columns (F.normalize(x, 1), aae.py:132-133).
// A row is spread over gridDim.x workgroups, `cc` columns each (100 rows x 100 000 items: 21 x 100 workgroups of 4 waves - the
// Box-Muller logf / cosf make the pass VALU-bound, and one 1024-thread workgroup per row would leave most of the chip idle).
// Pass 1 (this kernel) writes the noise of its columns - zeros in the padding columns [N, ldx) - and the sum of their |noise| to
// part[b][chunk]; without normalisation it also adds the row's entries that fall into its columns, and is the whole prelude.
__global__ __launch_bounds__(256) void dense_noise_gen_kernel(BatchView bv, float scale, int N, int normalize, int cc, int row0,
                                                              uint64_t seed, const long long* __restrict__ step_ctr,
                                                              float* __restrict__ X, int ldx, float* __restrict__ part) {
    __shared__ float red[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int c0 = blockIdx.x * cc, c1 = min(c0 + cc, ldx);
    const uint64_t k = dae_stream_key(seed, (uint64_t)*step_ctr, kDaeGaussStream);
    const uint32_t grow = (uint32_t)(row0 + b);
    float* row = X + (size_t)b * ldx;
    float acc = 0.f;
    for (int n = c0 + tid; n < c1; n += 256) {
        const float x = n < N ? dae_noise_cell(k, grow, n, scale) : 0.f;
        row[n] = x;
        acc += fabsf(x);
    }
    if (normalize) {
        acc = wave_sum(acc);
        if ((tid & 63) == 0) red[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0) part[b * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
        return;
    }
    __syncthreads();
    const int dc = bv.doc(b);
    const int64_t lo = bv.indptr[dc], hi = bv.indptr[dc + 1];
    for (int64_t e = lo + tid; e < hi; e += 256) {
        const int j = bv.indices[e];
        if (j >= c0 && j < c1) row[j] += bv.values[e];           // (column ids are unique within a row)
    }
}

// Pass 2 (normalisation only): the row's L1 norm = the chunk sums of |noise| in chunk order + sum over the row's entries of
// |noise_j + v_j| - |noise_j| with noise_j drawn again (a row has tens of entries; no workgroup reads a column another one writes),
// then the workgroup adds the entries of its own columns and scales its columns - the second and last pass over X.
// Every workgroup of a row forms the same norm from the same values in the same order.
__global__ __launch_bounds__(256) void dense_noise_finish_kernel(BatchView bv, float scale, int N, int cc, int row0, uint64_t seed,
                                                                 const long long* __restrict__ step_ctr, float* __restrict__ X,
                                                                 int ldx, const float* __restrict__ part) {
    __shared__ float red[4];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int c0 = blockIdx.x * cc, c1 = min(min(c0 + cc, ldx), N);
    const uint64_t k = dae_stream_key(seed, (uint64_t)*step_ctr, kDaeGaussStream);
    const uint32_t grow = (uint32_t)(row0 + b);
    float* row = X + (size_t)b * ldx;
    const int dc = bv.doc(b);
    const int64_t lo = bv.indptr[dc], hi = bv.indptr[dc + 1];
    float corr = 0.f;
    for (int64_t e = lo + tid; e < hi; e += 256) {
        const int j = bv.indices[e];
        const float x = dae_noise_cell(k, grow, j, scale), v = bv.values[e];
        corr += fabsf(__fadd_rn(x, v)) - fabsf(x);
        if (j >= c0 && j < c1) row[j] += v;
    }
    corr = wave_sum(corr);
    if (lane == 0) red[tid >> 6] = corr;
    __syncthreads();                                            // (also: the entries added above are in place for the scaling below)
    const float base = wave_sum(lane < (int)gridDim.x ? part[b * gridDim.x + lane] : 0.f);      // gridDim.x <= kDaeChunksMax = 64
    const float l1 = base + ((red[0] + red[1]) + (red[2] + red[3]));
    const float sc = 1.f / fmaxf(l1, 1e-12f);
    for (int n = c0 + tid; n < c1; n += 256) row[n] *= sc;
}

}  // namespace aae
