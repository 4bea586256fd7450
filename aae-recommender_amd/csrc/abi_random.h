// Entry points of the random baseline (randrank.h): the dense score block, and lists / ranks of draws that are regenerated where
// they are needed - no score matrix, no scratch.  Handle-free like the pop calls: every buffer is the caller's, every launch goes
// to the caller's stream, nothing synchronises.
// (one of the parts of aae_abi.hip's translation unit: included there in order, not on its own)
#pragma once

namespace {

// everything a call can be refused for by its numbers, before anything touches the device.  rows: what the message calls n_rows
int rand_check(const char* who, int64_t draw, int64_t row0, int32_t bits, int32_t n_items, int64_t n_rows, const char* rows) {
    const std::string w(who);
    if (n_items <= 0) return fail(AAE_EINVAL, w + ": n_items must be positive");
    if (bits < 1 || bits > 24) return fail(AAE_EINVAL, w + ": bits must be in [1, 24]");
    if (draw < 0) return fail(AAE_EINVAL, w + ": draw is negative");
    if (row0 < 0) return fail(AAE_EINVAL, w + ": row0 is negative");
    if (n_rows < 0) return fail(AAE_EINVAL, w + ": " + rows + " is negative");
    if (row0 + n_rows > ((int64_t)1 << 31)) return fail(AAE_EINVAL, w + ": row0 + " + rows + " exceeds 2^31");
    return AAE_OK;
}

int rand_check_batch(const char* who, const aae_batch* batch) {
    if (!batch || !batch->indptr_dev || !batch->indices_dev) return fail(AAE_EINVAL, std::string(who) + ": batch pointers are NULL");
    return AAE_OK;
}

RandArgs rand_args(uint64_t seed, int64_t draw, int64_t row0, int32_t bits, int32_t n_items) {
    return RandArgs{seed, (uint64_t)draw, (uint32_t)row0, (int)bits, (int)n_items};
}

}  // namespace

extern "C" {

int aae_rand_scores(uint64_t seed, int64_t draw, int64_t row0, int32_t bits, int32_t n_items, int32_t n_rows, float* out_dev,
                    int64_t ld, void* stream) {
    TRY(rand_check("aae_rand_scores", draw, row0, bits, n_items, n_rows, "n_rows"));
    if (!out_dev) return fail(AAE_EINVAL, "aae_rand_scores: out_dev is NULL");
    if (ld < n_items) return fail(AAE_EINVAL, "aae_rand_scores: ld < n_items");
    if (n_rows == 0) return AAE_OK;
    const dim3 grid((unsigned)(((int64_t)n_items + kRandNT - 1) / kRandNT), (unsigned)std::min<int32_t>(n_rows, kRandScoreRows));
    hipLaunchKernelGGL(pick_rand_scores(), grid, dim3(kRandNT), 0, S(stream), rand_args(seed, draw, row0, bits, n_items), (int)n_rows,
                       out_dev, (long long)ld);
    LAUNCHCHK("rand_scores");
    return AAE_OK;
}

int aae_rand_topk(uint64_t seed, int64_t draw, int64_t row0, int32_t bits, int32_t n_items, const aae_batch* batch, int32_t k,
                  int32_t exclude_known, int32_t* idx_out_dev, float* val_out_dev, void* stream) {
    TRY(rand_check_batch("aae_rand_topk", batch));
    TRY(rand_check("aae_rand_topk", draw, row0, bits, n_items, batch->n_rows, "batch->n_rows"));
    if (k < 1 || k > kRandKMax || k > n_items) return fail(AAE_EINVAL, "aae_rand_topk: k must be in [1, min(1024, n_items)]");
    if (!idx_out_dev) return fail(AAE_EINVAL, "aae_rand_topk: idx_out_dev is NULL");
    if (batch->n_rows == 0) return AAE_OK;
    hipLaunchKernelGGL(pick_rand_topk(), dim3((unsigned)batch->n_rows), dim3(kRandNT), 0, S(stream),
                       rand_args(seed, draw, row0, bits, n_items), rank_view(batch), (int)exclude_known, (int)k,
                       reinterpret_cast<int*>(idx_out_dev), val_out_dev);
    LAUNCHCHK("rand_topk");
    return AAE_OK;
}

int aae_rand_ranks(uint64_t seed, int64_t draw, int64_t row0, int32_t bits, int32_t n_items, const aae_batch* batch,
                   const aae_batch* truth, int32_t exclude_known, int32_t* ranks_out_dev, void* stream) {
    TRY(rand_check_batch("aae_rand_ranks", batch));
    TRY(rand_check("aae_rand_ranks", draw, row0, bits, n_items, batch->n_rows, "batch->n_rows"));
    TRY(rank_check_truth("aae_rand_ranks", batch->n_rows, truth));
    if (truth->max_row_nnz < 0) return fail(AAE_EINVAL, "aae_rand_ranks: truth->max_row_nnz is negative");
    if (truth->max_row_nnz > kRandTruthMax) return fail(AAE_EINVAL, "aae_rand_ranks: truth->max_row_nnz exceeds 4096 held-out items a row");
    if (!ranks_out_dev) return fail(AAE_EINVAL, "aae_rand_ranks: ranks_out_dev is NULL");
    if (batch->n_rows == 0) return AAE_OK;
    int cap = 1;                                                // (max_row_nnz = 0, unknown: room for the longest row there may be)
    const int longest = truth->max_row_nnz > 0 ? truth->max_row_nnz : kRandTruthMax;
    while (cap < longest) cap <<= 1;
    hipLaunchKernelGGL(pick_rand_ranks(), dim3((unsigned)batch->n_rows), dim3(kRandNT), (uint32_t)rand_ranks_lds_bytes(cap), S(stream),
                       rand_args(seed, draw, row0, bits, n_items), rank_view(batch), rank_view(truth), (int)exclude_known, cap,
                       reinterpret_cast<int*>(ranks_out_dev));
    LAUNCHCHK("rand_ranks");
    return AAE_OK;
}

}  // extern "C"
