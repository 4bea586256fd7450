// Entry points of the most-popular baseline (popular.h): the item counts of a training matrix, and lists / ranks from ONE item
// order shared by every row - no score matrix, no scratch.  Handle-free like the cooc calls: every buffer is the caller's, every
// launch (and the memset that zeroes the counts) goes to the caller's stream, nothing synchronises.
// (one of the parts of aae_abi.hip's translation unit: included there in order, not on its own)
#pragma once

namespace {

// everything a ranking call can be refused for before anything touches the device
int pop_check(const char* who, const aae_popular* pop, const aae_batch* batch) {
    const std::string w(who);
    if (!pop || !pop->counts_dev || !pop->order_dev || !pop->pos_dev) return fail(AAE_EINVAL, w + ": pop or one of its pointers is NULL");
    if (pop->n_items <= 0) return fail(AAE_EINVAL, w + ": n_items must be positive");
    if (!batch || !batch->indptr_dev || !batch->indices_dev) return fail(AAE_EINVAL, w + ": batch pointers are NULL");
    if (batch->n_rows < 0) return fail(AAE_EINVAL, w + ": batch->n_rows is negative");
    return AAE_OK;
}

PopView pop_view(const aae_popular* pop) { return PopView{pop->counts_dev, pop->order_dev, pop->pos_dev, pop->n_items}; }
unsigned pop_grid(int32_t n_rows) { return (unsigned)(((int64_t)n_rows + kPopRows - 1) / kPopRows); }

}  // namespace

extern "C" {

int aae_pop_counts(const aae_cooc* X, int32_t n_items, int32_t* counts_dev, void* stream) {
    if (!X || !X->indptr_dev || !X->indices_dev || !X->values_dev) return fail(AAE_EINVAL, "aae_pop_counts: X or one of its pointers is NULL");
    if (n_items <= 0) return fail(AAE_EINVAL, "aae_pop_counts: n_items must be positive");
    if (X->n_rows < 0) return fail(AAE_EINVAL, "aae_pop_counts: X->n_rows is negative");
    if (!counts_dev) return fail(AAE_EINVAL, "aae_pop_counts: counts_dev is NULL");
    hipStream_t s = S(stream);
    HIPCHK(hipMemsetAsync(counts_dev, 0, (size_t)n_items * sizeof(int32_t), s));
    if (X->n_rows == 0) return AAE_OK;
    const CoocView V{X->indptr_dev, X->indices_dev, X->values_dev, X->n_rows};
    hipLaunchKernelGGL(pick_pop_counts(), dim3(kPopCountBlocks), dim3(kPopNT), 0, s, V, (int)n_items, reinterpret_cast<int*>(counts_dev));
    LAUNCHCHK("pop_counts");
    return AAE_OK;
}

int aae_pop_topk(const aae_popular* pop, const aae_batch* batch, int32_t k, int32_t exclude_known, int32_t* idx_out_dev,
                 float* val_out_dev, void* stream) {
    TRY(pop_check("aae_pop_topk", pop, batch));
    if (k < 1 || k > pop->n_items) return fail(AAE_EINVAL, "aae_pop_topk: k must be in [1, n_items]");
    TRY(rank_check_lists("aae_pop_topk", idx_out_dev, val_out_dev));
    if (batch->n_rows == 0) return AAE_OK;
    hipLaunchKernelGGL(pick_pop_topk(), dim3(pop_grid(batch->n_rows)), dim3(kPopNT), 0, S(stream), pop_view(pop), rank_view(batch),
                       (int)exclude_known, (int)k, reinterpret_cast<int*>(idx_out_dev), val_out_dev);
    LAUNCHCHK("pop_topk");
    return AAE_OK;
}

int aae_pop_ranks(const aae_popular* pop, const aae_batch* batch, const aae_batch* truth, int32_t exclude_known,
                  int32_t* ranks_out_dev, void* stream) {
    TRY(pop_check("aae_pop_ranks", pop, batch));
    TRY(rank_check_truth("aae_pop_ranks", batch->n_rows, truth));
    if (!ranks_out_dev) return fail(AAE_EINVAL, "aae_pop_ranks: ranks_out_dev is NULL");
    if (batch->n_rows == 0) return AAE_OK;
    hipLaunchKernelGGL(pick_pop_ranks(), dim3(pop_grid(batch->n_rows)), dim3(kPopNT), 0, S(stream), pop_view(pop), rank_view(batch),
                       rank_view(truth), (int)exclude_known, reinterpret_cast<int*>(ranks_out_dev));
    LAUNCHCHK("pop_ranks");
    return AAE_OK;
}

}  // extern "C"
