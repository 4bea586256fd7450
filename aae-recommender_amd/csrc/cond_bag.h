// Bags of embedding rows on the device: EmbeddingBagCondition (reference aaerec/condition.py:372-394, nn.EmbeddingBag in its
// sum / mean / max modes) and CategoricalCondition(reduce="max") (condition.py:397-508, nn.Embedding(padding_idx=0) followed
// by hid.max(1)[0]).  cond_embed.h's sum / mean with a free padding row and the two max reductions.
//
//   encode   out[r][0:dim] = reduce over the slots w of row r of table[idx[r][w]]
//   update   the reduction's backward and the optimiser step (cat_update_kernel's SparseAdam, cat_dense_adam_kernel)
//
// padding_idx -1: no padding row (nn.EmbeddingBag's default; index 0 is an ordinary, trainable row); >= 0: that row is left
// out of the reduction and receives no gradient.  An index outside [0, vocab) is handled like a padding slot.
//   kBagSum         sum of the bag
//   kBagMeanWidth   sum / width, padding counted                (hid.mean(1))
//   kBagMeanCount   sum / number of non-padding slots, empty bag -> 0     (nn.EmbeddingBag(mode="mean"))
//   kBagMaxPad0     column-wise maximum; a padding slot is a candidate of value 0, so a row shorter than the padded width
//                   gives max(..., 0) and an all-padding row 0          (hid.max(1)[0] over nn.Embedding(padding_idx=0))
//   kBagMax         column-wise maximum of the non-padding slots, empty bag -> 0    (nn.EmbeddingBag(mode="max"))
// Tie rule of the two max modes: the gradient of (row r, column d) goes to the FIRST slot of row r that attains the maximum
// in column d (slot order, strict >); in kBagMaxPad0 to nobody when that slot is a padding slot.
//
// CONTRACT ON THE CALLER: the update recomputes the winners from the table, so nothing may modify the table between the
// encode and the update of a step (no argmax buffer crosses the step).  Inside the update the gradient launch only reads the
// table: in the max modes every optimiser (SparseAdam too) runs in a launch of its own from the [vocab][dim] gradient scratch.
//
// As in cat_update_kernel: one wavefront per index slot, lanes over columns (4 per lane, dim <= 256), no float atomics - the
// first slot that names a table row owns it, sums the contributions of every slot naming it in slot order and applies the
// optimiser to that row, so results do not depend on scheduling.  The duplicate scan is quadratic in rows * width.
#pragma once
#include "cond_embed.h"

namespace aae {

enum { kBagSum = 0, kBagMeanWidth = 1, kBagMeanCount = 2, kBagMaxPad0 = 3, kBagMax = 4 };

// a slot that takes part as a table row (neither padding nor out of range)
__device__ __forceinline__ bool bag_live(int j, int vocab, int pad) { return j >= 0 && j < vocab && j != pad; }

// Column `col` of row `ri` ([width] indices): the reduced value; *win = the first slot attaining the maximum (max modes; -1:
// none, or - kBagMaxPad0 - a padding slot), *cnt = the number of live slots.
__device__ __forceinline__ float bag_reduce_col(const float* __restrict__ table, int vocab, int dim, const int* __restrict__ ri,
                                                int width, int reduce, int pad, int col, int* win, int* cnt) {
    float acc = 0.f;
    int n = 0, best = -1;
    bool have = false;
    for (int w = 0; w < width; ++w) {
        const int j = ri[w];
        const bool live = bag_live(j, vocab, pad);
        n += live;
        if (reduce < kBagMaxPad0) {
            if (live) acc += table[(size_t)j * dim + col];
            continue;
        }
        if (!live && reduce == kBagMax) continue;
        const float t = live ? table[(size_t)j * dim + col] : 0.f;
        if (!have || t > acc) { acc = t; best = live ? w : -1; have = true; }
    }
    *win = best; *cnt = n;
    if (reduce == kBagMeanWidth) return acc / (float)width;
    if (reduce == kBagMeanCount) return n ? acc / (float)n : 0.f;
    return acc;
}

__global__ void __launch_bounds__(64)
bag_encode_kernel(const float* __restrict__ table, int vocab, int dim, const int* __restrict__ idx, int width, int reduce,
                  int pad, float* __restrict__ out, long long ldo) {
    const int r = blockIdx.x, col = blockIdx.y * 64 + threadIdx.x;
    if (col >= dim) return;
    int win, cnt;
    out[(size_t)r * ldo + col] = bag_reduce_col(table, vocab, dim, idx + (size_t)r * width, width, reduce, pad, col, &win, &cnt);
}

struct BagUpdate {
    CatUpdate c;                // c.mean is unused
    int reduce, pad;
};

// torch.optim.SparseAdam on one element, in cat_update_kernel's operation order
__device__ __forceinline__ void bag_sparse_adam(const CatUpdate& a, size_t o, float g) {
    const float m_old = a.m[o], v_old = a.v[o];
    const float mu = (g - m_old) * 0.1f;
    const float vu = (g * g - v_old) * 0.001f;
    const float m_new = m_old + mu, v_new = v_old + vu;
    a.m[o] = m_new; a.v[o] = v_new;
    a.table[o] += a.neg_step_size * (m_new / (sqrtf(v_new) + 1e-8f));
}

__global__ void __launch_bounds__(64 * kCatWaves)
bag_update_kernel(BagUpdate u) {
    const CatUpdate& a = u.c;
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * kCatWaves + (threadIdx.x >> 6);      // this wavefront's index slot
    const int n = a.rows * a.width;
    if (e >= n) return;
    const int j = a.idx[e];
    if (!bag_live(j, a.vocab, u.pad)) return;
    // an earlier slot with the same row owns it
    int dup = 0;
    for (int e2 = lane; e2 < e; e2 += 64) dup |= (a.idx[e2] == j);
    if (__any(dup)) return;
    // gradient of row j: every slot naming it, in slot order
    float g[kCatMaxDim / 64];
#pragma unroll
    for (int k = 0; k < kCatMaxDim / 64; ++k) g[k] = 0.f;
    for (int base = e & ~63; base < n; base += 64) {
        const int e2 = base + lane;
        const int hit = (e2 >= e && e2 < n) ? (a.idx[e2] == j) : 0;
        unsigned long long mask = __ballot(hit);
        while (mask) {
            const int s = base + __builtin_ctzll(mask);
            mask &= mask - 1;
            const int b = s / a.width, w = s - b * a.width;
            const int* ri = a.idx + (size_t)b * a.width;
            int live = 0;                                            // kBagMeanCount's divisor (>= 1: slot s is live)
            if (u.reduce == kBagMeanCount)
                for (int w2 = 0; w2 < a.width; ++w2) live += bag_live(ri[w2], a.vocab, u.pad);
#pragma unroll
            for (int k = 0; k < kCatMaxDim / 64; ++k) {
                const int col = lane + 64 * k;
                if (col >= a.dim) continue;
                const float dv = a.d[(size_t)b * a.ldd + col];
                if (u.reduce == kBagSum) g[k] += dv;
                else if (u.reduce == kBagMeanWidth) g[k] += dv / (float)a.width;
                else if (u.reduce == kBagMeanCount) g[k] += dv / (float)live;
                else {                                               // the winner, recomputed from the (unmodified) table
                    int win, cnt;
                    bag_reduce_col(a.table, a.vocab, a.dim, ri, a.width, u.reduce, u.pad, col, &win, &cnt);
                    if (win == w) g[k] += dv;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kCatMaxDim / 64; ++k) {
        const int col = lane + 64 * k;
        if (col >= a.dim) continue;
        const size_t o = (size_t)j * a.dim + col;
        // gdense set: the optimiser follows in a launch of its own - dense Adam over the whole table, or (max modes, whose
        // winners other wavefronts are still reading from the table) bag_sparse_adam_kernel
        if (a.gdense) a.gdense[o] = g[k];
        else bag_sparse_adam(a, o, g[k]);
    }
}

// SparseAdam of the max modes: the owners of bag_update_kernel apply their row's gradient from the scratch and clear it.
__global__ void __launch_bounds__(64 * kCatWaves)
bag_sparse_adam_kernel(BagUpdate u) {
    const CatUpdate& a = u.c;
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * kCatWaves + (threadIdx.x >> 6);
    if (e >= a.rows * a.width) return;
    const int j = a.idx[e];
    if (!bag_live(j, a.vocab, u.pad)) return;
    int dup = 0;
    for (int e2 = lane; e2 < e; e2 += 64) dup |= (a.idx[e2] == j);
    if (__any(dup)) return;
    for (int col = lane; col < a.dim; col += 64) {
        const size_t o = (size_t)j * a.dim + col;
        const float gi = a.gdense[o];
        a.gdense[o] = 0.f;
        bag_sparse_adam(a, o, gi);
    }
}

}  // namespace aae
