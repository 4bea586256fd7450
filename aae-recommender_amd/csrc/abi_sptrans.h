// Entry points of the device CSR transpose (sptrans.h): the Count pass and the Fill pass.  Handle-free like the cooc and spgemm
// calls: every buffer is the caller's, every launch (and the memset that zeroes a counter array) goes to the caller's stream,
// nothing synchronises - the exclusive scan between Count and Fill, and the allocation it sizes, are the caller's.
// (one of the parts of aae_abi.hip's translation unit: included there in order, not on its own)
#pragma once

static_assert(kSptransLds == AAE_SPTRANS_LDS, "include/aaerec_hip.h names the LDS segment limit of csrc/sptrans.h");

namespace {

int sptrans_check(const char* who, const int64_t* indptr_dev, const int32_t* indices_dev, int32_t n_rows, int32_t n_cols) {
    const std::string w(who);
    if (!indptr_dev || !indices_dev) return fail(AAE_EINVAL, w + ": indptr_dev / indices_dev is NULL");
    if (n_rows < 0 || n_cols < 0) return fail(AAE_EINVAL, w + ": n_rows / n_cols is negative");
    return AAE_OK;
}

}  // namespace

extern "C" {

int aae_csr_transpose_count(const int64_t* indptr_dev, const int32_t* indices_dev, int32_t n_rows, int32_t n_cols,
                            int64_t* col_nnz_dev, void* stream) {
    TRY(sptrans_check("aae_csr_transpose_count", indptr_dev, indices_dev, n_rows, n_cols));
    if (!col_nnz_dev) return fail(AAE_EINVAL, "aae_csr_transpose_count: col_nnz_dev is NULL");
    if (n_cols == 0) return AAE_OK;
    hipStream_t s = S(stream);
    if (hipMemsetAsync(col_nnz_dev, 0, (size_t)n_cols * sizeof(int64_t), s) != hipSuccess)
        return fail(AAE_EHIP, "aae_csr_transpose_count: hipMemsetAsync failed");
    if (n_rows == 0) return AAE_OK;
    SptransArgs g{};
    g.indptr = indptr_dev; g.indices = indices_dev; g.n_rows = n_rows; g.n_cols = n_cols;
    g.col_nnz = reinterpret_cast<unsigned long long*>(col_nnz_dev);
    hipLaunchKernelGGL(pick_sptrans_count(), dim3(kSptransCountBlocks), dim3(kSptransNT), 0, s, g);
    LAUNCHCHK("sptrans_count");
    return AAE_OK;
}

int aae_csr_transpose_fill(const int64_t* indptr_dev, const int32_t* indices_dev, const void* values_dev, int32_t n_rows,
                           int32_t n_cols, const int64_t* t_indptr_dev, int32_t* t_indices_dev, void* t_values_dev,
                           int64_t* cursor_dev, void* scratch_dev, int64_t scratch_pairs, int64_t nnz, void* stream) {
    TRY(sptrans_check("aae_csr_transpose_fill", indptr_dev, indices_dev, n_rows, n_cols));
    if (!values_dev) return fail(AAE_EINVAL, "aae_csr_transpose_fill: values_dev is NULL");
    if (!t_indptr_dev || !t_indices_dev || !t_values_dev) return fail(AAE_EINVAL, "aae_csr_transpose_fill: a pointer of the result is NULL");
    if (!cursor_dev) return fail(AAE_EINVAL, "aae_csr_transpose_fill: cursor_dev is NULL");
    if (nnz < 0 || scratch_pairs < 0) return fail(AAE_EINVAL, "aae_csr_transpose_fill: nnz / scratch_pairs is negative");
    // a segment longer than the LDS limit merges through the scratch; only a result of more entries can hold one
    if (nnz > kSptransLds && (!scratch_dev || scratch_pairs < nnz))
        return fail(AAE_EINVAL, "aae_csr_transpose_fill: a result of more than 4096 entries needs a scratch of nnz (row, value) pairs");
    if ((reinterpret_cast<uintptr_t>(scratch_dev) & 7) != 0) return fail(AAE_EINVAL, "aae_csr_transpose_fill: scratch_dev must be 8-byte aligned");
    if (n_rows == 0 || n_cols == 0) return AAE_OK;
    hipStream_t s = S(stream);
    if (hipMemsetAsync(cursor_dev, 0, (size_t)n_cols * sizeof(int64_t), s) != hipSuccess)
        return fail(AAE_EHIP, "aae_csr_transpose_fill: hipMemsetAsync failed");
    SptransArgs g{};
    g.indptr = indptr_dev; g.indices = indices_dev; g.values = static_cast<const uint32_t*>(values_dev);
    g.n_rows = n_rows; g.n_cols = n_cols;
    g.t_indptr = t_indptr_dev; g.t_indices = t_indices_dev; g.t_values = static_cast<uint32_t*>(t_values_dev);
    g.cursor = reinterpret_cast<unsigned long long*>(cursor_dev);
    g.scratch = static_cast<int2*>(scratch_dev); g.scratch_pairs = scratch_dev ? scratch_pairs : 0;
    hipLaunchKernelGGL(pick_sptrans_scatter(), dim3((unsigned)(((int64_t)n_rows + kSptransNT / 64 - 1) / (kSptransNT / 64))), dim3(kSptransNT), 0, s, g);
    LAUNCHCHK("sptrans_scatter");
    hipLaunchKernelGGL(pick_sptrans_sort(), dim3((unsigned)n_cols), dim3(kSptransNT), 0, s, g);
    LAUNCHCHK("sptrans_sort");
    return AAE_OK;
}

}  // extern "C"
