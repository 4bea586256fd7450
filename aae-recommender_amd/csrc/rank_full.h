// The rank of every held-out item in the FULL ranking of its row: what the unbounded metrics need ('mrr', 'map': the
// reference's drivers ask for them, evaluation.py:166-180) and all a bounded one needs too.  For each stored entry (row, t) of
// a ground-truth CSR: rank = 1 + #{items that come before t in the row's ordering} - the ordering of aae_predict_topk: known
// items are not rankable (exclude_known), the better score first, the smaller id at equal scores.  Only nnz(truth) integers
// leave the GPU; the [rows, n_items] matrix is never sorted, and in the fused form it never exists.
//
//   fused form (handles with rank_ok), behind the gather, the chain program and known_mask_kernel of a fused ranking
//   call (abi_rank.h).  The front end of rank_x3_kernel<NB, 1> - the kernel every list of k > 20 comes from, so the
//   logits carry the same bits as the ones those lists were ordered by - with two more epilogues, kFullSlots = 8 held-out
//   items per row and pair of launches:
//     1. rank_full_setup_kernel          the rows' next 8 held-out ids into tgt_i (-1: none), their counters zeroed
//     2. rank_x3_kernel<.., kRankPick>   a cell that is one of its row's 8 items stores its logit into tgt_v[row][slot]
//                                        (-inf when the item is a known one)
//     3. rank_x3_kernel<.., kRankCount>  every epilogue thread holds its row's 8 (logit, id) in registers; each of its four
//                                        cells per tile is compared with them: logit > l_t || (logit == l_t && item < t).
//                                        A known cell enters as -inf.  The 8 threads of a row add up by lane shuffles, one
//                                        integer atomicAdd per (row, slot, workgroup): the sums do not depend on order.
//     4. rank_full_finish_kernel         rank = 1 + count, written at the entry's place in CSR order
//   A row with MORE than 8 held-out items is answered by REPEATING 1-4 over the next groups of 8 slots (ceil(longest truth
//   row / 8) rounds per call, two passes over dec.lin3 each) - not by the dense form: the ranks of a call all come from the
//   same logits.
//   A held-out item that is itself a known item ranks behind every rankable item, among the known items by id:
//   n_rankable + 1 + #{known ids < t} - which is what the comparison above yields with known cells at -inf.
//   An id outside [0, n_items) gets rank 0.
//
//   dense form (every other handle; rows beyond the fused call's limit)
//     rank_full_dense_kernel             one workgroup per row of the [rows][N] score matrix in the scratch: known items masked
//                                        to -inf in place (as rank_long_dense_kernel), then 8 held-out items at a time counted
//                                        over the row - by score, then the smaller id.  Templated on the score type as
//                                        rank_long_dense_kernel (rank_long.h DenseScore): float, or the int32 co-occurrence scores.
// No float atomics, no inline assembly: integer counters in LDS / HBM and plain stores.
#pragma once
#include "rank_long.h"

namespace aae {

constexpr int kFullNT = 1024;

// Where the entries of call row `row` begin in the call's output (entries of the rows before it, CSR order).  The whole
// workgroup calls it; red: LDS for blockDim.x / 64 values; ends behind a barrier.
__device__ __forceinline__ long long truth_offset(const BatchView& tv, int row, long long* red) {
    if (!tv.rows) return tv.indptr[tv.row_start + row] - tv.indptr[tv.row_start];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (blockDim.x + 63) >> 6;
    long long sum = 0;
    for (int r = tid; r < row; r += blockDim.x) { const int dc = tv.rows[r]; sum += tv.indptr[dc + 1] - tv.indptr[dc]; }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    __syncthreads();
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    sum = 0;
    for (int w = 0; w < nw; ++w) sum += red[w];
    return sum;
}

// ---- fused form -------------------------------------------------------------------------------------------------
// One workgroup per row: slots [group * 8, group * 8 + 8) of the row's held-out items
__global__ __launch_bounds__(64) void rank_full_setup_kernel(BatchView tv, int n_items, int group, int* __restrict__ tgt_i,
                                                             float* __restrict__ tgt_v, int* __restrict__ tcount) {
    const int row = blockIdx.x, s = threadIdx.x;
    if (s >= kFullSlots) return;
    const int dc = tv.doc(row);
    const int64_t e = tv.indptr[dc] + (int64_t)group * kFullSlots + s;
    int t = e < tv.indptr[dc + 1] ? tv.indices[e] : -1;
    if (t < 0 || t >= n_items) t = -1;
    tgt_i[row * kFullSlots + s] = t;
    tgt_v[row * kFullSlots + s] = INFINITY;        // (nothing compares as before an unused slot)
    tcount[row * kFullSlots + s] = 0;
}

__global__ __launch_bounds__(256) void rank_full_finish_kernel(BatchView tv, int group, const int* __restrict__ tgt_i,
                                                               const int* __restrict__ tcount, int* __restrict__ ranks_out) {
    __shared__ long long red[4];
    const int row = blockIdx.x, s = threadIdx.x;
    const int dc = tv.doc(row);
    const int64_t lo = tv.indptr[dc], hi = tv.indptr[dc + 1];
    if (lo + (int64_t)group * kFullSlots >= hi) return;
    const long long off = truth_offset(tv, row, red);
    const int64_t j = (int64_t)group * kFullSlots + s;
    if (s < kFullSlots && lo + j < hi) ranks_out[off + j] = tgt_i[row * kFullSlots + s] >= 0 ? 1 + tcount[row * kFullSlots + s] : 0;
}

// ---- dense form -------------------------------------------------------------------------------------------------
// One workgroup per row of the score matrix (sigmoids): row `blockIdx.x` of the matrix is row `row0 + blockIdx.x` of the call
// (`kv`: its input rows, `tv`: its truth rows).
template <class SC>
__global__ __launch_bounds__(kFullNT) void rank_full_dense_kernel(SC* __restrict__ scores, int ld, int n_items, BatchView kv,
                                                                  BatchView tv, int row0, int exclude_known,
                                                                  int* __restrict__ ranks_out) {
    __shared__ long long red[kFullNT / 64];
    __shared__ int t_id[kFullSlots], t_cnt[kFullSlots];
    __shared__ SC t_sc[kFullSlots];
    using D = DenseScore<SC>;
    const int tid = threadIdx.x, row = row0 + blockIdx.x;
    SC* sc = scores + (size_t)blockIdx.x * ld;
    if (exclude_known) {
        const int dc = kv.doc(row);
        const int64_t lo = kv.indptr[dc], hi = kv.indptr[dc + 1];
        for (int64_t e = lo + tid; e < hi; e += kFullNT) {
            const int i = kv.indices[e];
            if (i >= 0 && i < n_items) sc[i] = D::lowest();
        }
    }
    const int dc = tv.doc(row);
    const int64_t lo = tv.indptr[dc], hi = tv.indptr[dc + 1];
    const long long off = truth_offset(tv, row, red);
    for (int64_t e0 = lo; e0 < hi; e0 += kFullSlots) {
        __syncthreads();                // (the mask is in place; the previous group's results are written)
        if (tid < kFullSlots) {
            int t = e0 + tid < hi ? tv.indices[e0 + tid] : -1;
            if (t < 0 || t >= n_items) t = -1;
            t_id[tid] = t; t_sc[tid] = t >= 0 ? sc[t] : D::highest(); t_cnt[tid] = 0;      // (nothing comes before an unused slot: its id is -1)
        }
        __syncthreads();
        int id[kFullSlots], cnt[kFullSlots]; SC ts[kFullSlots];
#pragma unroll
        for (int s = 0; s < kFullSlots; ++s) { id[s] = t_id[s]; ts[s] = t_sc[s]; cnt[s] = 0; }
        for (int i = tid; i < n_items; i += kFullNT) {
            const SC v = sc[i];
#pragma unroll
            for (int s = 0; s < kFullSlots; ++s) cnt[s] += (v > ts[s] || (v == ts[s] && i < id[s])) ? 1 : 0;
        }
#pragma unroll
        for (int s = 0; s < kFullSlots; ++s) {
            int c = cnt[s];
            for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
            if ((tid & 63) == 0 && c > 0) atomicAdd(&t_cnt[s], c);
        }
        __syncthreads();
        if (tid < kFullSlots && e0 + tid < hi) ranks_out[off + (e0 - lo) + tid] = t_id[tid] >= 0 ? 1 + t_cnt[tid] : 0;
    }
}

}  // namespace aae
