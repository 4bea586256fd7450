// Entry points of the truncated-SVD baseline (lowrank.h): scores alone, or scores into the caller's scratch followed by the
// dense ranking calls of abi_rank.h (dense_topk / dense_ranks) as they stand.  Handle-free like the cooc calls: every buffer is the
// caller's, every launch goes to the caller's stream, nothing synchronises.
// (one of the parts of aae_abi.hip's translation unit: included there in order, not on its own)
#pragma once

static_assert(kProjDimsMax == AAE_LOWRANK_DIMS_MAX, "include/aaerec_hip.h names the widest hidden vector of csrc/lowrank.h");

namespace {

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// everything a call can be refused for before anything touches the device (features: the rows the projection reads)
int lowrank_check(const char* who, const aae_lowrank* lr, int32_t n_items, const aae_batch* features, const float* hidden_dev,
                  int64_t hidden_ld, const float* scores_dev, int64_t ld) {
    const std::string w(who);
    if (!lr || !lr->vt_dev) return fail(AAE_EINVAL, w + ": lowrank or its table is NULL");
    if (lr->dims < 1 || lr->dims > kProjDimsMax) return fail(AAE_EINVAL, w + ": lowrank->dims must be in [1, 4096]");
    if (lr->n_features < 1) return fail(AAE_EINVAL, w + ": lowrank->n_features must be positive");
    if (lr->ld < (((int64_t)lr->dims + 3) & ~(int64_t)3) || (lr->ld & 3) || lr->ld > 0x7FFFFFFF || !aligned16(lr->vt_dev))
        return fail(AAE_EINVAL, w + ": the table's leading dimension (lowrank->ld) must be a multiple of 4 floats, at least dims rounded up to 4, "
                                    "and the table 16-byte aligned");
    if (n_items <= 0 || n_items > lr->n_features) return fail(AAE_EINVAL, w + ": n_items must be in [1, lowrank->n_features]");
    if (!features || !features->indptr_dev || !features->indices_dev || !features->values_dev) return fail(AAE_EINVAL, w + ": feature batch pointers are NULL");
    if (features->n_rows < 0) return fail(AAE_EINVAL, w + ": features->n_rows is negative");
    if (!hidden_dev) return fail(AAE_EINVAL, w + ": the hidden scratch is NULL");
    if (hidden_ld < lr->dims || (hidden_ld & 3) || hidden_ld > 0x7FFFFFFF || !aligned16(hidden_dev))
        return fail(AAE_EINVAL, w + ": the hidden scratch's leading dimension (hidden_ld) is smaller than dims, or not a multiple of 4 floats on a 16-byte aligned base");
    if (!scores_dev) return fail(AAE_EINVAL, w + ": the score matrix (scratch) is NULL");
    if (ld < n_items) return fail(AAE_EINVAL, w + ": the score matrix's leading dimension (scratch_ld) is smaller than n_items");
    if ((ld & 3) || ld > 0x7FFFFFFF || !aligned16(scores_dev))
        return fail(AAE_EINVAL, w + ": the score matrix's leading dimension must be a multiple of 4 floats below 2^31 on a 16-byte aligned base");
    return AAE_OK;
}
// the item rows of a ranking call: the known items, ids in [0, n_items)
int lowrank_check_items(const char* who, const aae_batch* features, const aae_batch* items) {
    const std::string w(who);
    if (!items || !items->indptr_dev || !items->indices_dev) return fail(AAE_EINVAL, w + ": item batch pointers are NULL");
    if (items->n_rows != features->n_rows) return fail(AAE_EINVAL, w + ": the item batch names another number of rows than the feature batch");
    return AAE_OK;
}

int lowrank_launch(const aae_lowrank* lr, int32_t n_items, const aae_batch* features, float* hidden_dev, int64_t hidden_ld,
                   float* scores_dev, int64_t ld, hipStream_t s) {
    const int rows = features->n_rows;
    const LowRankView V{lr->vt_dev, (long long)lr->ld, lr->n_features, lr->dims};
    hipLaunchKernelGGL(pick_lowrank_project(), dim3((unsigned)rows), dim3(lowrank_project_threads(lr->dims)), 0, s, V, rank_view(features),
                       hidden_dev, (long long)hidden_ld);
    LAUNCHCHK("lowrank_project");
    GemmShape g;
    g.A = hidden_dev; g.B = lr->vt_dev;
    g.M = rows; g.N = n_items; g.K = lr->dims;
    g.lda = (int)hidden_ld; g.ldb = (int)lr->ld;
    g.k_per_split = (lr->dims + 15) & ~15;          // split-K count 1: one k-ordered chain per score
    EpiStore epi; epi.out = scores_dev; epi.ld = (int)ld;
    const unsigned grid = gemm_remapped_grid(g, (n_items + 63) / 64, (rows + 63) / 64, 1);
    hipLaunchKernelGGL(pick_lowrank_gemm(), dim3(grid), dim3(256), 0, s, g, epi);
    LAUNCHCHK("lowrank reconstruction (gemm_f32)");
    return AAE_OK;
}

}  // namespace

extern "C" {

int aae_lowrank_scores(const aae_lowrank* lowrank, int32_t n_items, const aae_batch* features, float* hidden_dev, int64_t hidden_ld,
                       float* scores_dev, int64_t ld, void* stream) {
    TRY(lowrank_check("aae_lowrank_scores", lowrank, n_items, features, hidden_dev, hidden_ld, scores_dev, ld));
    if (features->n_rows == 0) return AAE_OK;
    return lowrank_launch(lowrank, n_items, features, hidden_dev, hidden_ld, scores_dev, ld, S(stream));
}

int aae_spmm_f32(const aae_batch* rows, const float* dense_dev, int64_t ld, int32_t n_cols, int32_t width, float* out_dev,
                 int64_t ld_out, void* stream) {
    const std::string w("aae_spmm_f32");
    if (!rows || !rows->indptr_dev || !rows->indices_dev || !rows->values_dev) return fail(AAE_EINVAL, w + ": row batch pointers are NULL");
    if (rows->n_rows < 0) return fail(AAE_EINVAL, w + ": rows->n_rows is negative");
    if (width < 1 || width > kProjDimsMax) return fail(AAE_EINVAL, w + ": width must be in [1, 4096]");
    if (n_cols < 1) return fail(AAE_EINVAL, w + ": n_cols must be positive");
    if (!dense_dev || !out_dev) return fail(AAE_EINVAL, w + ": dense_dev / out_dev is NULL");
    if (ld < (((int64_t)width + 3) & ~(int64_t)3) || (ld & 3) || ld > 0x7FFFFFFF || !aligned16(dense_dev))
        return fail(AAE_EINVAL, w + ": the dense operand's leading dimension (ld) must be a multiple of 4 floats, at least width rounded up to 4, "
                                    "and the operand 16-byte aligned");
    if (ld_out < width || (ld_out & 3) || ld_out > 0x7FFFFFFF || !aligned16(out_dev))
        return fail(AAE_EINVAL, w + ": the result's leading dimension (ld_out) is smaller than width, or not a multiple of 4 floats on a 16-byte aligned base");
    if (rows->n_rows == 0) return AAE_OK;
    const LowRankView V{dense_dev, (long long)ld, n_cols, width};
    hipLaunchKernelGGL(pick_lowrank_project(), dim3((unsigned)rows->n_rows), dim3(lowrank_project_threads(width)), 0, S(stream), V,
                       rank_view(rows), out_dev, (long long)ld_out);
    LAUNCHCHK("spmm_f32 (lowrank_project)");
    return AAE_OK;
}

int aae_lowrank_topk(const aae_lowrank* lowrank, int32_t n_items, const aae_batch* features, const aae_batch* items, int32_t k,
                     int32_t exclude_known, float* hidden_dev, int64_t hidden_ld, float* scratch_dev, int64_t scratch_ld,
                     int32_t* idx_out_dev, float* val_out_dev, void* stream) {
    const char* who = "aae_lowrank_topk";
    TRY(lowrank_check(who, lowrank, n_items, features, hidden_dev, hidden_ld, scratch_dev, scratch_ld));
    TRY(lowrank_check_items(who, features, items));
    TRY(rank_check_k(who, k, n_items));
    TRY(rank_check_lists(who, idx_out_dev, val_out_dev));
    if (features->n_rows == 0) return AAE_OK;
    TRY(lowrank_launch(lowrank, n_items, features, hidden_dev, hidden_ld, scratch_dev, scratch_ld, S(stream)));
    return dense_topk(scratch_dev, scratch_ld, n_items, rank_view(items), items->n_rows, k, exclude_known, idx_out_dev, val_out_dev, S(stream));
}

int aae_lowrank_ranks(const aae_lowrank* lowrank, int32_t n_items, const aae_batch* features, const aae_batch* items,
                      const aae_batch* truth, int32_t exclude_known, float* hidden_dev, int64_t hidden_ld, float* scratch_dev,
                      int64_t scratch_ld, int32_t* ranks_out_dev, void* stream) {
    const char* who = "aae_lowrank_ranks";
    TRY(lowrank_check(who, lowrank, n_items, features, hidden_dev, hidden_ld, scratch_dev, scratch_ld));
    TRY(lowrank_check_items(who, features, items));
    TRY(rank_check_truth(who, features->n_rows, truth));
    if (!ranks_out_dev) return fail(AAE_EINVAL, std::string(who) + ": ranks_out_dev is NULL");
    if (features->n_rows == 0) return AAE_OK;
    TRY(lowrank_launch(lowrank, n_items, features, hidden_dev, hidden_ld, scratch_dev, scratch_ld, S(stream)));
    return dense_ranks(scratch_dev, scratch_ld, n_items, rank_view(items), rank_view(truth), items->n_rows, exclude_known, ranks_out_dev, S(stream));
}

}  // extern "C"
