// Entry points of the item co-occurrence baseline (cooc.h): scores alone, or scores into the caller's scratch followed by the
// dense ranking calls of abi_rank.h (dense_topk / dense_ranks).  Each call exists for both score types of those kernels (SC: float, and
// int32_t behind the _i32 names - the same checks, the same launches, the integer members of the three kernels).  Handle-free:
// every buffer is the caller's, every launch goes to the caller's stream, nothing synchronises.
// (one of the parts of aae_abi.hip's translation unit: included there in order, not on its own)
#pragma once

static_assert(kCoocTile == AAE_COOC_TILE, "include/aaerec_hip.h names the tile width of csrc/cooc.h");

namespace {

// everything a call can be refused for before anything touches the device
int cooc_check(const char* who, const aae_cooc* cooc, int32_t n_items, const aae_batch* batch, const void* scores_dev, int64_t ld) {
    const std::string w(who);
    if (!cooc || !cooc->indptr_dev || !cooc->indices_dev || !cooc->values_dev) return fail(AAE_EINVAL, w + ": cooc or one of its pointers is NULL");
    if (n_items <= 0) return fail(AAE_EINVAL, w + ": n_items must be positive");
    if (cooc->n_rows < 0) return fail(AAE_EINVAL, w + ": cooc->n_rows is negative");
    if (!batch || !batch->indptr_dev || !batch->indices_dev || !batch->values_dev) return fail(AAE_EINVAL, w + ": batch pointers are NULL");
    if (batch->n_rows < 0) return fail(AAE_EINVAL, w + ": batch->n_rows is negative");
    if (!scores_dev) return fail(AAE_EINVAL, w + ": the score matrix (scratch) is NULL");
    if (ld < n_items) return fail(AAE_EINVAL, w + ": the score matrix's leading dimension (scratch_ld) is smaller than n_items");
    if (ld > 0x7FFFFFFF) return fail(AAE_EINVAL, w + ": the score matrix's leading dimension does not fit 31 bits");
    const int64_t ntiles = ((int64_t)n_items + kCoocTile - 1) / kCoocTile;
    if (batch->n_rows * ntiles > 0x7FFFFFFF) return fail(AAE_EINVAL, w + ": rows x item tiles exceed one launch's grid");
    return AAE_OK;
}

template <class SC>
int cooc_launch(const aae_cooc* cooc, int32_t n_items, const aae_batch* batch, SC* scores_dev, int64_t ld, hipStream_t s) {
    const int ntiles = (n_items + kCoocTile - 1) / kCoocTile;
    const CoocView C{cooc->indptr_dev, cooc->indices_dev, cooc->values_dev, cooc->n_rows};
    hipLaunchKernelGGL(pick_cooc_scores<SC>(), dim3((unsigned)(batch->n_rows * ntiles)), dim3(kCoocNT), 0, s, C, (int)n_items, ntiles,
                       rank_view(batch), scores_dev, (long long)ld);
    LAUNCHCHK("cooc_scores");
    return AAE_OK;
}

template <class SC>
int cooc_scores(const char* who, const aae_cooc* cooc, int32_t n_items, const aae_batch* batch, SC* scores_dev, int64_t ld, void* stream) {
    TRY(cooc_check(who, cooc, n_items, batch, scores_dev, ld));
    if (batch->n_rows == 0) return AAE_OK;
    return cooc_launch(cooc, n_items, batch, scores_dev, ld, S(stream));
}

template <class SC>
int cooc_topk(const char* who, const aae_cooc* cooc, int32_t n_items, const aae_batch* batch, int32_t k, int32_t exclude_known,
              SC* scratch_dev, int64_t scratch_ld, int32_t* idx_out_dev, float* val_out_dev, void* stream) {
    TRY(cooc_check(who, cooc, n_items, batch, scratch_dev, scratch_ld));
    TRY(rank_check_k(who, k, n_items));
    TRY(rank_check_lists(who, idx_out_dev, val_out_dev));
    if (batch->n_rows == 0) return AAE_OK;
    TRY(cooc_launch(cooc, n_items, batch, scratch_dev, scratch_ld, S(stream)));
    return dense_topk(scratch_dev, scratch_ld, n_items, rank_view(batch), batch->n_rows, k, exclude_known, idx_out_dev, val_out_dev, S(stream));
}

template <class SC>
int cooc_ranks(const char* who, const aae_cooc* cooc, int32_t n_items, const aae_batch* batch, const aae_batch* truth, int32_t exclude_known,
               SC* scratch_dev, int64_t scratch_ld, int32_t* ranks_out_dev, void* stream) {
    TRY(cooc_check(who, cooc, n_items, batch, scratch_dev, scratch_ld));
    TRY(rank_check_truth(who, batch->n_rows, truth));
    if (!ranks_out_dev) return fail(AAE_EINVAL, std::string(who) + ": ranks_out_dev is NULL");
    if (batch->n_rows == 0) return AAE_OK;
    TRY(cooc_launch(cooc, n_items, batch, scratch_dev, scratch_ld, S(stream)));
    return dense_ranks(scratch_dev, scratch_ld, n_items, rank_view(batch), rank_view(truth), batch->n_rows, exclude_known, ranks_out_dev, S(stream));
}

}  // namespace

extern "C" {

int aae_cooc_scores(const aae_cooc* cooc, int32_t n_items, const aae_batch* batch, float* scores_dev, int64_t ld, void* stream) {
    return cooc_scores("aae_cooc_scores", cooc, n_items, batch, scores_dev, ld, stream);
}
int aae_cooc_scores_i32(const aae_cooc* cooc, int32_t n_items, const aae_batch* batch, int32_t* scores_dev, int64_t ld, void* stream) {
    return cooc_scores("aae_cooc_scores_i32", cooc, n_items, batch, scores_dev, ld, stream);
}

int aae_cooc_topk(const aae_cooc* cooc, int32_t n_items, const aae_batch* batch, int32_t k, int32_t exclude_known,
                  float* scratch_dev, int64_t scratch_ld, int32_t* idx_out_dev, float* val_out_dev, void* stream) {
    return cooc_topk("aae_cooc_topk", cooc, n_items, batch, k, exclude_known, scratch_dev, scratch_ld, idx_out_dev, val_out_dev, stream);
}
int aae_cooc_topk_i32(const aae_cooc* cooc, int32_t n_items, const aae_batch* batch, int32_t k, int32_t exclude_known,
                      int32_t* scratch_dev, int64_t scratch_ld, int32_t* idx_out_dev, float* val_out_dev, void* stream) {
    return cooc_topk("aae_cooc_topk_i32", cooc, n_items, batch, k, exclude_known, scratch_dev, scratch_ld, idx_out_dev, val_out_dev, stream);
}

int aae_cooc_ranks(const aae_cooc* cooc, int32_t n_items, const aae_batch* batch, const aae_batch* truth, int32_t exclude_known,
                   float* scratch_dev, int64_t scratch_ld, int32_t* ranks_out_dev, void* stream) {
    return cooc_ranks("aae_cooc_ranks", cooc, n_items, batch, truth, exclude_known, scratch_dev, scratch_ld, ranks_out_dev, stream);
}
int aae_cooc_ranks_i32(const aae_cooc* cooc, int32_t n_items, const aae_batch* batch, const aae_batch* truth, int32_t exclude_known,
                       int32_t* scratch_dev, int64_t scratch_ld, int32_t* ranks_out_dev, void* stream) {
    return cooc_ranks("aae_cooc_ranks_i32", cooc, n_items, batch, truth, exclude_known, scratch_dev, scratch_ld, ranks_out_dev, stream);
}

}  // extern "C"
