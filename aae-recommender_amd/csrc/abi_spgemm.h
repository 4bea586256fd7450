// Entry points of the exact int32 sparse product (spgemm.h): the product bound of every row, the Count pass, the Fill pass.
// Handle-free like the cooc calls: every buffer is the caller's, every launch goes to the caller's stream, nothing synchronises -
// the exclusive scan between Count and Fill, and the allocation it sizes, are the caller's.
// (one of the parts of aae_abi.hip's translation unit: included there in order, not on its own)
#pragma once

static_assert(kSpgemmHashProducts == AAE_SPGEMM_HASH_PRODUCTS, "include/aaerec_hip.h names the bin edge of csrc/spgemm.h");
static_assert(kSpgemmStage == AAE_SPGEMM_STAGE, "include/aaerec_hip.h names the staging piece of csrc/spgemm.h");

namespace {

// everything a call can be refused for before anything touches the device
int spgemm_check(const char* who, const aae_cooc* A, const aae_cooc* B, int64_t cols, const void* u_dev) {
    const std::string w(who);
    for (const aae_cooc* M : {A, B})
        if (!M || !M->indptr_dev || !M->indices_dev || !M->values_dev) return fail(AAE_EINVAL, w + ": an operand or one of its pointers is NULL");
    if (A->n_rows < 0 || B->n_rows < 0) return fail(AAE_EINVAL, w + ": an operand's n_rows is negative");
    if (cols < 0 || cols > 0x7FFFFFFF) return fail(AAE_EINVAL, w + ": the column count must be in [0, 2^31)");
    if (!u_dev) return fail(AAE_EINVAL, w + ": u_dev is NULL");
    return AAE_OK;
}

SpgemmArgs spgemm_args(const aae_cooc* A, const aae_cooc* B, int32_t n, const int64_t* u_dev) {
    SpgemmArgs g{};
    g.A = CoocView{A->indptr_dev, A->indices_dev, A->values_dev, A->n_rows};
    g.B = CoocView{B->indptr_dev, B->indices_dev, B->values_dev, B->n_rows};
    g.p = B->n_rows; g.n = n; g.u = u_dev;
    return g;
}

int spgemm_launch(bool fill, const SpgemmArgs& g, hipStream_t s) {
    hipLaunchKernelGGL(pick_spgemm_hash(fill), dim3((unsigned)g.A.n_rows), dim3(kSpgemmHashNT), 0, s, g);
    LAUNCHCHK("spgemm_hash");
    hipLaunchKernelGGL(pick_spgemm_tile(fill), dim3((unsigned)g.A.n_rows), dim3(kSpgemmTileNT), 0, s, g);
    LAUNCHCHK("spgemm_tile");
    return AAE_OK;
}

}  // namespace

extern "C" {

int aae_spgemm_i32_bound(const aae_cooc* A, const aae_cooc* B, int32_t p, int64_t* u_dev, void* stream) {
    TRY(spgemm_check("aae_spgemm_i32_bound", A, B, p, u_dev));
    if (p > B->n_rows) return fail(AAE_EINVAL, "aae_spgemm_i32_bound: p exceeds the rows of B");
    if (A->n_rows == 0) return AAE_OK;
    const CoocView a{A->indptr_dev, A->indices_dev, A->values_dev, A->n_rows}, b{B->indptr_dev, B->indices_dev, B->values_dev, B->n_rows};
    hipLaunchKernelGGL(spgemm_bound_kernel, dim3((unsigned)(((int64_t)A->n_rows + 3) / 4)), dim3(256), 0, S(stream), a, b, (int)p, u_dev);
    LAUNCHCHK("spgemm_bound");
    return AAE_OK;
}

int aae_spgemm_i32_count(const aae_cooc* A, const aae_cooc* B, int32_t n, const int64_t* u_dev, int64_t* row_nnz_dev, void* stream) {
    TRY(spgemm_check("aae_spgemm_i32_count", A, B, n, u_dev));
    if (!row_nnz_dev) return fail(AAE_EINVAL, "aae_spgemm_i32_count: row_nnz_dev is NULL");
    if (A->n_rows == 0) return AAE_OK;
    SpgemmArgs g = spgemm_args(A, B, n, u_dev);
    g.row_nnz = row_nnz_dev;
    return spgemm_launch(false, g, S(stream));
}

int aae_spgemm_i32_fill(const aae_cooc* A, const aae_cooc* B, int32_t n, const int64_t* u_dev, const int64_t* indptr_dev,
                        int32_t* indices_dev, int32_t* values_dev, void* stream) {
    TRY(spgemm_check("aae_spgemm_i32_fill", A, B, n, u_dev));
    if (!indptr_dev || !indices_dev || !values_dev) return fail(AAE_EINVAL, "aae_spgemm_i32_fill: a pointer of the result is NULL");
    if (A->n_rows == 0) return AAE_OK;
    SpgemmArgs g = spgemm_args(A, B, n, u_dev);
    g.indptr = indptr_dev; g.indices = indices_dev; g.values = values_dev;
    return spgemm_launch(true, g, S(stream));
}

}  // extern "C"
