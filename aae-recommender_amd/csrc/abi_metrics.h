// Entry points of the ranking metrics (rank_metrics.h): per-row values from held-out ranks, their (mean, std), and the bridge from
// top-k lists to ranks.  Handle-free like the popular calls: every buffer is the caller's, every launch goes to the caller's
// stream, nothing synchronises.
// (one of the parts of aae_abi.hip's translation unit: included there in order, not on its own)
#pragma once

namespace {

unsigned metric_grid(int32_t n_rows) { return (unsigned)(((int64_t)n_rows + kMetricRows - 1) / kMetricRows); }

}  // namespace

extern "C" {

int aae_metric_rows(const aae_rank_rows* rows, const aae_metric_spec* specs, int32_t n_metrics, const double* discounts_dev,
                    int32_t n_discounts, double* per_row_dev, int64_t ld, void* stream) {
    if (!rows || !rows->indptr_dev || !rows->ranks_dev) return fail(AAE_EINVAL, "aae_metric_rows: rows or one of its pointers is NULL");
    if (rows->n_rows < 0) return fail(AAE_EINVAL, "aae_metric_rows: rows->n_rows is negative");
    if (!specs) return fail(AAE_EINVAL, "aae_metric_rows: specs is NULL");
    if (n_metrics < 1 || n_metrics > AAE_METRIC_MAX) return fail(AAE_EINVAL, "aae_metric_rows: n_metrics must be in [1, AAE_METRIC_MAX]");
    if (n_discounts < 0) return fail(AAE_EINVAL, "aae_metric_rows: n_discounts is negative");
    if (!per_row_dev) return fail(AAE_EINVAL, "aae_metric_rows: per_row_dev is NULL");
    if (ld < rows->n_rows) return fail(AAE_EINVAL, "aae_metric_rows: ld is smaller than rows->n_rows");
    MetricSpecs sp;
    sp.n = n_metrics;
    for (int q = 0; q < n_metrics; ++q) {
        const int kind = specs[q].kind, k = specs[q].k;
        if (kind < 0 || kind >= kMetKinds) return fail(AAE_EINVAL, "aae_metric_rows: unknown metric kind");
        if (k < 0 || k == AAE_RANK_ABSENT) return fail(AAE_EINVAL, "aae_metric_rows: k must be in [0, AAE_RANK_ABSENT)");
        if (k == 0 && kind != AAE_METRIC_MRR && kind != AAE_METRIC_MAP)
            return fail(AAE_EINVAL, "aae_metric_rows: k = 0 (unbounded) is defined for mrr and map only");
        if (kind == AAE_METRIC_NDCG && !discounts_dev) return fail(AAE_EINVAL, "aae_metric_rows: an ndcg spec needs discounts_dev");
        if (kind == AAE_METRIC_NDCG && k > n_discounts) return fail(AAE_EINVAL, "aae_metric_rows: an ndcg spec's k exceeds n_discounts");
        sp.kind[q] = kind; sp.k[q] = k;
    }
    for (int q = n_metrics; q < kMetricMax; ++q) { sp.kind[q] = 0; sp.k[q] = 0; }
    if (rows->n_rows == 0) return AAE_OK;
    const MetricRowsArgs a{rows->indptr_dev, rows->ranks_dev, rows->n_rows, discounts_dev, n_discounts, per_row_dev, (long long)ld};
    hipLaunchKernelGGL(pick_metric_rows(), dim3(metric_grid(rows->n_rows)), dim3(kMetricNT), 0, S(stream), a, sp);
    LAUNCHCHK("metric_rows");
    return AAE_OK;
}

int aae_metric_finish(const double* per_row_dev, int64_t ld, int32_t n_rows, int32_t n_metrics, double* out_dev, void* stream) {
    if (!per_row_dev || !out_dev) return fail(AAE_EINVAL, "aae_metric_finish: per_row_dev / out_dev is NULL");
    if (n_rows < 0) return fail(AAE_EINVAL, "aae_metric_finish: n_rows is negative");
    if (n_metrics < 1 || n_metrics > AAE_METRIC_MAX) return fail(AAE_EINVAL, "aae_metric_finish: n_metrics must be in [1, AAE_METRIC_MAX]");
    if (ld < n_rows) return fail(AAE_EINVAL, "aae_metric_finish: ld is smaller than n_rows");
    hipLaunchKernelGGL(pick_metric_finish(), dim3(n_metrics), dim3(kMetricNT), 0, S(stream), per_row_dev, (long long)ld, (int)n_rows, out_dev);
    LAUNCHCHK("metric_finish");
    return AAE_OK;
}

int aae_ranks_from_lists(const int32_t* ids_dev, int64_t ld, int32_t k, const aae_batch* truth, int32_t* ranks_out_dev, void* stream) {
    if (!ids_dev) return fail(AAE_EINVAL, "aae_ranks_from_lists: ids_dev is NULL");
    if (k < 1) return fail(AAE_EINVAL, "aae_ranks_from_lists: k must be positive");
    if (ld < k) return fail(AAE_EINVAL, "aae_ranks_from_lists: ld is smaller than k");
    if (!truth || !truth->indptr_dev || !truth->indices_dev) return fail(AAE_EINVAL, "aae_ranks_from_lists: truth pointers are NULL");
    if (truth->n_rows < 0) return fail(AAE_EINVAL, "aae_ranks_from_lists: truth->n_rows is negative");
    // (rank_check_truth of the sibling calls compares the truth's rows with an input batch's: there is none here, the truth names
    //  the rows of the call itself.  rows_dev is a device array - its entries are the caller's, as in every aae_batch)
    if (!truth->rows_dev && truth->row_start < 0) return fail(AAE_EINVAL, "aae_ranks_from_lists: truth->row_start is negative");
    if (!ranks_out_dev) return fail(AAE_EINVAL, "aae_ranks_from_lists: ranks_out_dev is NULL");
    if (truth->n_rows == 0) return AAE_OK;
    hipLaunchKernelGGL(pick_ranks_from_lists(), dim3(metric_grid(truth->n_rows)), dim3(kMetricNT), 0, S(stream), ids_dev, (long long)ld,
                       (int)k, rank_view(truth), reinterpret_cast<int*>(ranks_out_dev));
    LAUNCHCHK("ranks_from_lists");
    return AAE_OK;
}

}  // extern "C"
