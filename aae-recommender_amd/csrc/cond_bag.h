// Bags of embedding rows on the device: the trainable conditions of the reference (aaerec/condition.py) - CategoricalCondition
// (397-508: nn.Embedding(padding_idx=0) followed by .sum(1) / .mean(1) / .max(1)[0]) and EmbeddingBagCondition (372-394:
// nn.EmbeddingBag in its sum / mean / max modes).  This file states their arithmetic ONCE - the reduction of a column
// (bag_reduce_col), what an entry adds to its table row's gradient (bag_grad_add), SparseAdam on an element (bag_sparse_adam)
// and the two ways a row's gradient leaves a wavefront (bag_write_row, bag_apply_row) - and holds the kernels over a padded
// [rows][width] index block; cond_csr.h runs the same helpers over a resident CSR.
//
//   encode   out[r][0:dim] = reduce over the slots w of row r of table[idx[r][w]]
//   update   the reduction's backward and the optimiser step (SparseAdam here, cond_embed.h's cat_dense_adam_kernel)
//   renorm   nn.Embedding's max_norm: every table row the input names whose p-norm exceeds max_norm is scaled onto it, once,
//            in a launch of its own in front of the encode (bag_row_renorm)
//
// padding_idx -1: no padding row (nn.EmbeddingBag's default; index 0 is an ordinary, trainable row); >= 0: that row is left
// out of the reduction and receives no gradient.  An index outside [0, vocab) is handled like a padding slot.
//   kBagSum         sum of the bag
//   kBagMeanWidth   sum / width, padding counted                (hid.mean(1))
//   kBagMeanCount   sum / number of non-padding slots, empty bag -> 0     (nn.EmbeddingBag(mode="mean"))
//   kBagMaxPad0     column-wise maximum; a padding slot is a candidate of value 0, so a row shorter than the padded width
//                   gives max(..., 0) and an all-padding row 0          (hid.max(1)[0] over nn.Embedding(padding_idx=0))
//   kBagMax         column-wise maximum of the non-padding slots, empty bag -> 0    (nn.EmbeddingBag(mode="max"))
// aae_cat_* is kBagSum / kBagMeanWidth at padding row 0 through these kernels.
// Tie rule of the two max modes: the gradient of (row r, column d) goes to the FIRST slot of row r that attains the maximum
// in column d (slot order, strict >); in kBagMaxPad0 to nobody when that slot is a padding slot.
//
// CONTRACT ON THE CALLER: the update recomputes the winners from the table, so nothing may modify the table between the
// encode and the update of a step (no argmax buffer crosses the step).  Inside the update the gradient launch only reads the
// table: in the max modes every optimiser (SparseAdam too) runs in a launch of its own from the [vocab][dim] gradient scratch.
//
// A batch holds rows * width indices (a few hundred): one wavefront per index slot, lanes over columns (4 per lane, dim <=
// 256), no float atomics - the first slot that names a table row owns it, sums the contributions of every slot naming it in
// slot order (the sparse gradient's coalesce()) and hands the row on, so results do not depend on scheduling.  The duplicate
// scan is quadratic in rows * width.
//
// scale_grad_by_freq (BagTable::by_freq): the owner has visited every slot naming its row, so it knows their number - the
// whole batch's, every bag's, the losers of the max modes included - and divides the summed gradient by it
// (bag_freq_scale: one division per element, behind the sum).
//
// Contraction is part of the bits: bag_reduce_col and bag_grad_add keep a per-sample weight's product a multiply of its own
// (fp contract off), bag_sparse_adam stands outside any such pragma.  tests/golden/cond_bits.json records the result.
#pragma once
#include "cond_embed.h"

namespace aae {

enum { kBagSum = 0, kBagMeanWidth = 1, kBagMeanCount = 2, kBagMaxPad0 = 3, kBagMax = 4 };

// a slot that takes part as a table row (neither padding nor out of range)
__device__ __forceinline__ bool bag_live(int j, int vocab, int pad) { return j >= 0 && j < vocab && j != pad; }

// Column `col` of a row: its `len` entries ri[] (wt: their weights, kBagSum only; NULL: none) followed by dead slots up to
// `width` (a padded block: len == width).  Dead slots change nothing but kBagMeanWidth's divisor and, behind the entries,
// give kBagMaxPad0 one candidate of value 0.  Returns the reduced value; *win = the first entry attaining the maximum (max
// modes; -1: none, or - kBagMaxPad0 - a dead slot), *cnt = the number of live entries.
__device__ __forceinline__ float bag_reduce_col(const float* __restrict__ table, int vocab, int dim, const int* __restrict__ ri,
                                                const float* __restrict__ wt, long long len, int width, int reduce, int pad,
                                                int col, int* win, int* cnt) {
#pragma clang fp contract(off)
    float acc = 0.f;
    int n = 0, best = -1;
    bool have = false;
    for (long long w = 0; w < len; ++w) {
        const int j = ri[w];
        const bool live = bag_live(j, vocab, pad);
        n += live;
        if (reduce < kBagMaxPad0) {
            if (live) {
                const float t = table[(size_t)j * dim + col];
                acc += wt ? wt[w] * t : t;
            }
            continue;
        }
        if (!live && reduce == kBagMax) continue;
        const float t = live ? table[(size_t)j * dim + col] : 0.f;
        if (!have || t > acc) { acc = t; best = live ? (int)w : -1; have = true; }
    }
    if (reduce == kBagMaxPad0 && len < (long long)width && (!have || 0.f > acc)) { acc = 0.f; best = -1; }
    *win = best; *cnt = n;
    if (reduce == kBagMeanWidth) return acc / (float)width;
    if (reduce == kBagMeanCount) return n ? acc / (float)n : 0.f;
    return acc;
}

// The backward of bag_reduce_col for one live entry and one column: adds to g what the entry contributes to its table row's
// gradient.  dv: dout of the entry's row; live: the row's live entries (kBagMeanCount); winner: the entry is the column's *win
// (max modes); weighted: the entry has the weight wt (kBagSum), multiply-then-add.
__device__ __forceinline__ void bag_grad_add(float& g, int reduce, float dv, int width, int live, bool winner, bool weighted,
                                             float wt) {
#pragma clang fp contract(off)
    if (reduce == kBagSum) g += weighted ? wt * dv : dv;
    else if (reduce == kBagMeanWidth) g += dv / (float)width;
    else if (reduce == kBagMeanCount) g += dv / (float)live;
    else if (winner) g += dv;
}

// the table side of an update
struct BagTable {
    float* table; float* m; float* v;
    float* gdense;              // [vocab][dim] gradient scratch (all zero between steps) the optimiser follows from in a launch of
                                // its own: dense Adam, and SparseAdam in the max modes; NULL: SparseAdam inside the gradient launch
    const float* d; long long ldd;      // dout [rows][>= dim]
    int vocab, dim, reduce, pad;
    float neg_step_size;        // SparseAdam: -(lr * sqrt(1 - b2^t) / (1 - b1^t))
    int by_freq;                // scale_grad_by_freq: a row's gradient is divided by the number of entries of the batch naming it
};

// torch.optim.SparseAdam on one element, in its operation order (torch/optim/_functional.py sparse_adam)
__device__ __forceinline__ void bag_sparse_adam(const BagTable& a, size_t o, float g) {
    const float m_old = a.m[o], v_old = a.v[o];
    const float mu = (g - m_old) * 0.1f;
    const float vu = (g * g - v_old) * 0.001f;
    const float m_new = m_old + mu, v_new = v_old + vu;
    a.m[o] = m_new; a.v[o] = v_new;
    a.table[o] += a.neg_step_size * (m_new / (sqrtf(v_new) + 1e-8f));
}

// the owner of table row j hands on the gradient it summed (lane: columns lane + 64 k): to the scratch, or to SparseAdam
__device__ __forceinline__ void bag_write_row(const BagTable& a, int j, int lane, const float (&g)[kCatMaxDim / 64]) {
#pragma unroll
    for (int k = 0; k < kCatMaxDim / 64; ++k) {
        const int col = lane + 64 * k;
        if (col >= a.dim) continue;
        const size_t o = (size_t)j * a.dim + col;
        if (a.gdense) a.gdense[o] = g[k];
        else bag_sparse_adam(a, o, g[k]);
    }
}

// SparseAdam of the max modes (whose winners other wavefronts were still reading from the table during the gradient launch):
// the owner of table row j applies the row from the scratch and clears it
__device__ __forceinline__ void bag_apply_row(const BagTable& a, int j, int lane) {
    for (int col = lane; col < a.dim; col += 64) {
        const size_t o = (size_t)j * a.dim + col;
        const float gi = a.gdense[o];
        a.gdense[o] = 0.f;
        bag_sparse_adam(a, o, gi);
    }
}

// scale_grad_by_freq: the gradient the owner summed over the `count` (>= 1) entries naming its row, divided by their number
__device__ __forceinline__ void bag_freq_scale(const BagTable& a, float (&g)[kCatMaxDim / 64], int count) {
    if (!a.by_freq) return;
    const float n = (float)count;
#pragma unroll
    for (int k = 0; k < kCatMaxDim / 64; ++k) g[k] = g[k] / n;
}

// ---- max_norm ------------------------------------------------------------------------------------------------------------
enum { kBagNormInf = 0, kBagNormL1 = 1, kBagNormL2 = 2 };

// The p-norm of a table row over a wavefront (lane: columns lane + 64 k, ascending k), fp32: the lanes' partial sums of |x|^p
// (p = 1, 2) or maxima (p = inf), folded by the xor butterfly 32, 16, .. 1 - one fixed order, the same value in every lane -
// and, p = 2, the square root.
__device__ __forceinline__ float bag_row_norm(const float* __restrict__ row, int dim, int lane, int norm_type) {
#pragma clang fp contract(off)
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < kCatMaxDim / 64; ++k) {
        const int col = lane + 64 * k;
        if (col >= dim) continue;
        const float x = row[col];
        if (norm_type == kBagNormL2) acc += x * x;
        else if (norm_type == kBagNormL1) acc += fabsf(x);
        else acc = fmaxf(acc, fabsf(x));
    }
    for (int d = 32; d > 0; d >>= 1) {
        const float y = __shfl_xor(acc, d);
        acc = norm_type == kBagNormInf ? fmaxf(acc, y) : acc + y;
    }
    return norm_type == kBagNormL2 ? sqrtf(acc) : acc;
}

// torch's embedding_renorm_ on the row its owner holds: norm > max_norm (strictly) scales the row by max_norm / (norm + 1e-7)
__device__ __forceinline__ void bag_row_renorm(float* __restrict__ table, int dim, int j, int lane, float max_norm, int norm_type) {
    float* row = table + (size_t)j * dim;
    const float norm = bag_row_norm(row, dim, lane, norm_type);
    if (!(norm > max_norm)) return;
    const float scale = max_norm / (norm + 1e-7f);
    for (int col = lane; col < dim; col += 64) row[col] = row[col] * scale;
}

// ---- the padded source: idx [rows][width] --------------------------------------------------------------------------------
struct BagPadded { const int* idx; int rows, width; };

__global__ void __launch_bounds__(64)
bag_encode_kernel(const float* __restrict__ table, int vocab, int dim, const int* __restrict__ idx, int width, int reduce,
                  int pad, float* __restrict__ out, long long ldo) {
    const int r = blockIdx.x, col = blockIdx.y * 64 + threadIdx.x;
    if (col >= dim) return;
    int win, cnt;
    out[(size_t)r * ldo + col] = bag_reduce_col(table, vocab, dim, idx + (size_t)r * width, nullptr, width, width, reduce, pad,
                                                col, &win, &cnt);
}

// the table row index slot e owns under the padding row `pad`: the slot's row if it is live and no earlier slot names it, else
// -1 (pad -1: every row of the table can be owned - the renorm's rule, which scales a padding row too)
__device__ __forceinline__ int bag_first_slot(const BagPadded& s, int e, int lane, int vocab, int pad) {
    if (e >= s.rows * s.width) return -1;
    const int j = s.idx[e];
    if (!bag_live(j, vocab, pad)) return -1;
    int dup = 0;
    for (int e2 = lane; e2 < e; e2 += 64) dup |= (s.idx[e2] == j);
    return __any(dup) ? -1 : j;
}

__device__ __forceinline__ int bag_owned_row(const BagTable& a, const BagPadded& s, int e, int lane) {
    return bag_first_slot(s, e, lane, a.vocab, a.pad);
}

__global__ void __launch_bounds__(64 * kCatWaves)
bag_renorm_kernel(float* __restrict__ table, int vocab, int dim, BagPadded s, float max_norm, int norm_type) {
    const int lane = threadIdx.x & 63;
    const int j = bag_first_slot(s, blockIdx.x * kCatWaves + (threadIdx.x >> 6), lane, vocab, -1);
    if (j >= 0) bag_row_renorm(table, dim, j, lane, max_norm, norm_type);
}

__global__ void __launch_bounds__(64 * kCatWaves)
bag_update_kernel(BagTable a, BagPadded s) {
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * kCatWaves + (threadIdx.x >> 6);      // this wavefront's index slot
    const int n = s.rows * s.width;
    const int j = bag_owned_row(a, s, e, lane);
    if (j < 0) return;
    // gradient of row j: every slot naming it, in slot order
    float g[kCatMaxDim / 64];
#pragma unroll
    for (int k = 0; k < kCatMaxDim / 64; ++k) g[k] = 0.f;
    int named = 0;                                                   // slots naming row j (scale_grad_by_freq)
    for (int base = e & ~63; base < n; base += 64) {
        const int e2 = base + lane;
        const int hit = (e2 >= e && e2 < n) ? (s.idx[e2] == j) : 0;
        unsigned long long mask = __ballot(hit);
        named += __builtin_popcountll(mask);
        while (mask) {
            const int slot = base + __builtin_ctzll(mask);
            mask &= mask - 1;
            const int b = slot / s.width, w = slot - b * s.width;
            const int* ri = s.idx + (size_t)b * s.width;
            int live = 0;                                            // kBagMeanCount's divisor (>= 1: the slot is live)
            if (a.reduce == kBagMeanCount)
                for (int w2 = 0; w2 < s.width; ++w2) live += bag_live(ri[w2], a.vocab, a.pad);
#pragma unroll
            for (int k = 0; k < kCatMaxDim / 64; ++k) {
                const int col = lane + 64 * k;
                if (col >= a.dim) continue;
                int win = -1, cnt;                                   // the winner, recomputed from the (unmodified) table
                if (a.reduce >= kBagMaxPad0) bag_reduce_col(a.table, a.vocab, a.dim, ri, nullptr, s.width, s.width, a.reduce, a.pad, col, &win, &cnt);
                bag_grad_add(g[k], a.reduce, a.d[(size_t)b * a.ldd + col], s.width, live, win == w, false, 0.f);
            }
        }
    }
    bag_freq_scale(a, g, named);
    bag_write_row(a, j, lane, g);
}

__global__ void __launch_bounds__(64 * kCatWaves)
bag_apply_kernel(BagTable a, BagPadded s) {
    const int lane = threadIdx.x & 63;
    const int j = bag_owned_row(a, s, blockIdx.x * kCatWaves + (threadIdx.x >> 6), lane);
    if (j >= 0) bag_apply_row(a, j, lane);
}

}  // namespace aae
