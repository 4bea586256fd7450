// What the trainable conditions share with the rest of the library: the limits of their kernels, torch.optim.Adam over a whole
// embedding table, and the weighted bag of pretrained vectors.  The trainable conditions themselves - CategoricalCondition and
// EmbeddingBagCondition (reference aaerec/condition.py:372-508), lookup + reduction, backward and optimiser step - are
// cond_bag.h (padded index blocks; aae_cat_* is its sum / mean at padding row 0) and cond_csr.h (a resident CSR).
#pragma once
#include "device_common.h"

namespace aae {

constexpr int kCatMaxDim = 256;       // 4 columns per lane
constexpr int kCatWaves = 4;          // wavefronts per workgroup

// torch.optim.Adam over the whole table (nn.Embedding(sparse=False)): rows without a gradient still decay their
// moments and move.  Consumes and clears the gradient scratch.
__global__ void __launch_bounds__(256)
cat_dense_adam_kernel(float* __restrict__ table, float* __restrict__ m, float* __restrict__ v, float* __restrict__ g,
                      size_t n, OptScalars sc) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float gi = g[i];
    if (gi != 0.f) g[i] = 0.f;
    float p = table[i], mi = m[i], vi = v[i];
    // exact sqrt / division here (adam_update's 1-ulp approximations buy nothing on a table this small)
    mi = mi + 0.1f * (gi - mi);
    vi = vi * 0.999f + (0.001f * gi) * gi;
    const float denom = sqrtf(vi) / sc.bc2_sqrt + 1e-8f;
    p = p + sc.neg_step_size * (mi / denom);
    table[i] = p; m[i] = mi; v[i] = vi;
}

// Weighted bag of embedded words (reference ub.py:52-57, `sparse_scores @ self.embedding`): out[r] = sum over the
// CSR entries e of row r of values[e] * table[indices[e]], entries in CSR order (scipy's order).  One workgroup per
// document, a thread per column (coalesced 1 KB row segments); the TF-IDF rows of a title hold 5-20 words.
__global__ void __launch_bounds__(256)
csr_embed_kernel(const long long* __restrict__ indptr, const int* __restrict__ indices, const float* __restrict__ values,
                 const float* __restrict__ table, int n_table_rows, int dim, long long ldt, float* __restrict__ out,
                 long long ldo) {
    const int r = blockIdx.x;
    const long long e0 = indptr[r], e1 = indptr[r + 1];
    for (int col = threadIdx.x; col < dim; col += 256) {
        float acc = 0.f;
        for (long long e = e0; e < e1; ++e) {
            const int j = indices[e];
            if (j >= 0 && j < n_table_rows) acc += values[e] * table[(size_t)j * ldt + col];
        }
        out[(size_t)r * ldo + col] = acc;
    }
}

}  // namespace aae
